// Connected components of a CHUNK of bit planes of different sizes (s2d_plane_components_ragged) and the cleanup of such planes
// on top of them (s2d_plane_clean_ragged): s2d_amd/plane_components.py, DESIGN.md section 1.  The planes are the flat buffer the
// ragged RLE decode fills (rle_ragged.hip): plane int64 [P][4] = {word0, H, W, 0}, pixel i = y*W + x of a plane in word i / 32, bit
// i % 32 (bitplane.h), so rows are not word-aligned.  The masks of a chunk overlap, so there is no index map to label: every plane
// is labelled on its own, and one launch covers all of them.  The cleanup rule is this project's own: the reference cleans nothing.
//
// The structure is that of index_components.hip, with the tile-local labelling and the union-find bodies shared (components.h).
// Every kernel runs over a host-built tile table, tiles int32 [n_tiles][3] = {plane, tile row, tile column}: a chunk holds thousands
// of planes of a few tiles each, so the grid is 1-D over the table and a workgroup reads its plane's geometry from the plane table.
//   1. pc_tile_kernel     a CC_TH x CC_TW tile per workgroup: the tile's row words (row_word: pixels at and beyond W are 0) become
//                         one byte per pixel in LDS -- 1 where the bit equals `value` --, then cc_tile_label.  With value = 0 the
//                         row mask is applied AFTER the complement: padding bits and everything outside the plane join nothing.
//   2. pc_merge_kernel    the pixels of the tile's first column and first row join their neighbours in the tiles to the left and
//                         above, through agent-scope atomics only; a link only ever decreases.
//   3. pc_flatten_kernel  labels = 1 + root, tile-local counts move to the root (one integer atomic per tile-local component); for
//                         the hole rule a border pixel sets the sign bit of its root's area word (areas are < 2^31, so the OR and
//                         the adds commute).
// Element 32 * word0 + i of parent / labels / area belongs to pixel i of the plane: 64-bit indices, a chunk passes 2^31 elements.
// The cleanup copies the planes to `out` (padding zeroed) and then only clears or sets bits there with atomicAnd / atomicOr from the
// labels: it never reads a bit it may have changed, so `out` may be `bits`.  No workgroup waits for another; integer atomics only.
#include "bitplane.h"
#include "components.h"

namespace {

constexpr unsigned PC_BORDER = 0x80000000u;                              // area word of a root: its component touches the plane's border

struct PcTile {
    PlaneRow q;
    int f, x0, y0, tw, th;
    bool ok;
};

// the workgroup's row of the tile table; a row that names no tile of a plane the buffer holds is skipped (uniform over the workgroup)
__device__ __forceinline__ PcTile pc_tile(const int *__restrict__ tiles, const long *__restrict__ plane, int P, long total_words)
{
    const int *t = tiles + 3L * blockIdx.x;
    PcTile c;
    c.f = t[0];
    const long y0 = (long)t[1] * CC_TH, x0 = (long)t[2] * CC_TW;
    c.ok = c.f >= 0 && c.f < P && y0 >= 0 && x0 >= 0;
    if (!c.ok) return c;
    c.q = plane_row(plane, c.f, total_words);
    c.ok = c.q.ok && y0 < c.q.H && x0 < c.q.W;
    if (!c.ok) return c;
    c.x0 = (int)x0; c.y0 = (int)y0;
    c.tw = min(CC_TW, c.q.W - c.x0); c.th = min(CC_TH, c.q.H - c.y0);
    return c;
}

// is pixel i of the plane one to label
__device__ __forceinline__ bool pc_pix(const uint32_t *pl, long i, unsigned value) { return ((pl[i >> 5] >> (i & 31)) & 1u) == value; }

// ---- launch 1 ----
__global__ __launch_bounds__(CC_THREADS) void pc_tile_kernel(const uint32_t *bits, const long *__restrict__ plane, int P, long total_words,
                                                             const int *__restrict__ tiles, unsigned value, int conn8, int *__restrict__ parent,
                                                             int *__restrict__ area)
{
    __shared__ unsigned ids32[CC_TILE / 4];
    __shared__ unsigned par[CC_TILE];
    __shared__ unsigned cnt[CC_TILE];
    const PcTile c = pc_tile(tiles, plane, P, total_words);
    if (!c.ok) return;
    const int tid = threadIdx.x, W = c.q.W;
    const uint32_t *pl = bits + c.q.word0;

    for (int i = tid; i < CC_TILE / 4; i += CC_THREADS) ids32[i] = 0u;
    __syncthreads();
    for (int it = tid; it < c.th * (CC_TW / 32); it += CC_THREADS) {
        const int row = it / (CC_TW / 32), k = c.x0 / 32 + it % (CC_TW / 32);
        const int n = W - 32 * k;
        if (n < 1) continue;
        const unsigned v = row_word(pl, c.q.wpp, c.y0 + row, W, k);
        const unsigned fg = value ? v : (~v & (n >= 32 ? 0xffffffffu : (1u << n) - 1u));
        unsigned *dst = ids32 + (row * CC_TW + 32 * (it % (CC_TW / 32))) / 4;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const unsigned x = (fg >> (4 * j)) & 0xfu;
            dst[j] = (x & 1u) | ((x & 2u) << 7) | ((x & 4u) << 14) | ((x & 8u) << 21);
        }
    }
    __syncthreads();

    const int ly = tid / (CC_TW / CC_PER), lx0 = (tid % (CC_TW / CC_PER)) * CC_PER;
    const unsigned i0 = ly * CC_TW + lx0;
    unsigned root[CC_PER];
    cc_tile_label(reinterpret_cast<const uint8_t *>(ids32), par, cnt, conn8, root);
    if (ly >= c.th) return;
    const long g0 = 32 * c.q.word0 + (long)(c.y0 + ly) * W + c.x0;
    for (int j = 0; j < CC_PER; ++j) {
        const int lx = lx0 + j;
        if (lx >= c.tw) break;
        const unsigned r = root[j];
        parent[g0 + lx] = r == CC_NONE ? -1 : (int)((long)(c.y0 + (int)(r / CC_TW)) * W + c.x0 + (int)(r % CC_TW));
        if (area) area[g0 + lx] = r == i0 + j ? (int)cnt[r] : 0;
    }
}

// ---- launch 2 ----
// the tile's first column joins the tile to the left, its first row the tile above.  As in cc_merge_kernel, a diagonal contact that
// crosses a vertical border belongs to the column part, the ones at tile corners included; the row part takes the diagonals that
// stay inside a tile column.  Where the straight neighbour is a pixel to label, the diagonals beside it are joined through it.
__global__ __launch_bounds__(CC_THREADS) void pc_merge_kernel(const uint32_t *bits, const long *__restrict__ plane, int P, long total_words,
                                                              const int *__restrict__ tiles, unsigned value, int conn8, int *parent)
{
    const PcTile c = pc_tile(tiles, plane, P, total_words);
    if (!c.ok) return;
    const int e = threadIdx.x, H = c.q.H, W = c.q.W;
    const uint32_t *pl = bits + c.q.word0;
    int *par = parent + 32 * c.q.word0;
    if (e < CC_TH) {
        if (c.x0 == 0 || e >= c.th) return;
        const int x = c.x0, y = c.y0 + e;
        const int p = y * W + x;
        if (!pc_pix(pl, p, value)) return;
        if (pc_pix(pl, p - 1, value)) {
            glb_union(par, p, p - 1);
        } else if (conn8) {
            if (y > 0 && pc_pix(pl, p - W - 1, value)) glb_union(par, p, p - W - 1);
            if (y + 1 < H && pc_pix(pl, (long)p + W - 1, value)) glb_union(par, p, p + W - 1);
        }
    } else if (e < CC_TH + CC_TW) {
        if (c.y0 == 0 || e - CC_TH >= c.tw) return;
        const int x = c.x0 + e - CC_TH, y = c.y0;
        const int p = y * W + x;
        if (!pc_pix(pl, p, value)) return;
        if (pc_pix(pl, p - W, value)) {
            glb_union(par, p, p - W);
        } else if (conn8) {
            if (x % CC_TW != 0 && pc_pix(pl, p - W - 1, value)) glb_union(par, p, p - W - 1);
            if ((x + 1) % CC_TW != 0 && x + 1 < W && pc_pix(pl, p - W + 1, value)) glb_union(par, p, p - W + 1);
        }
    }
}

// ---- launch 3 ----
__global__ __launch_bounds__(CC_THREADS) void pc_flatten_kernel(const long *__restrict__ plane, int P, long total_words,
                                                                const int *__restrict__ tiles, const int *__restrict__ parent,
                                                                int *__restrict__ labels, int *area, int mark_border)
{
    const PcTile c = pc_tile(tiles, plane, P, total_words);
    if (!c.ok) return;
    const int tid = threadIdx.x, H = c.q.H, W = c.q.W;
    const int ly = tid / (CC_TW / CC_PER), lx0 = (tid % (CC_TW / CC_PER)) * CC_PER;
    if (ly >= c.th) return;
    const long base = 32 * c.q.word0;
    const int y = c.y0 + ly;
    for (int j = 0; j < CC_PER; ++j) {
        const int lx = lx0 + j;
        if (lx >= c.tw) break;
        const int x = c.x0 + lx, q = y * W + x;
        const long t = base + q;
        int r = parent[t];
        if (r < 0) {
            labels[t] = 0;
            continue;
        }
        for (int nx; (nx = parent[base + r]) != r;) r = nx;
        labels[t] = r + 1;
        if (!area) continue;
        // area[t] != 0: t is a tile-local root, and only this thread touches the word unless it is the root (then the others add to it)
        if (r != q) {
            const int a = area[t];
            if (a) {
                atomicAdd(&area[base + r], a);
                area[t] = 0;
            }
        }
        if (mark_border && (y == 0 || y == H - 1 || x == 0 || x == W - 1)) {
            unsigned *w = reinterpret_cast<unsigned *>(&area[base + r]);
            if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & PC_BORDER)) atomicOr(w, PC_BORDER);
        }
    }
}

// ---- the cleanup ----
// out = bits with the padding bits of every plane's last word zeroed; a workgroup per plane.  A thread reads a word before it writes
// it, so out may be bits.
__global__ __launch_bounds__(256) void pc_copy_kernel(const uint32_t *bits, const long *__restrict__ plane, long total_words, uint32_t *out)
{
    const PlaneRow q = plane_row(plane, blockIdx.x, total_words);
    if (!q.ok) return;
    const int n = (int)((long)q.H * q.W - 32 * (q.wpp - 1));            // pixels of the last word, 1 .. 32
    for (long w = threadIdx.x; w < q.wpp; w += 256) {
        unsigned v = bits[q.word0 + w];
        if (w == q.wpp - 1 && n < 32) v &= (1u << n) - 1u;
        out[q.word0 + w] = v;
    }
}

// best[plane] = max over the plane's components of cc_key(area, first pixel).  A wave reduces its keys first and sends one atomic,
// unless the entry already beats it (the entry only grows): a checkerboard would otherwise queue H*W atomics on one address.
__global__ __launch_bounds__(CC_THREADS) void pc_best_kernel(const long *__restrict__ plane, int P, long total_words,
                                                             const int *__restrict__ tiles, const int *__restrict__ area,
                                                             unsigned long long *best)
{
    const PcTile c = pc_tile(tiles, plane, P, total_words);
    if (!c.ok) return;
    const int tid = threadIdx.x, W = c.q.W;
    const int ly = tid / (CC_TW / CC_PER), lx0 = (tid % (CC_TW / CC_PER)) * CC_PER;
    unsigned long long key = 0ull;
    if (ly < c.th) {
        const int q0 = (c.y0 + ly) * W + c.x0;
        for (int j = 0; j < CC_PER && lx0 + j < c.tw; ++j) {
            const int a = area[32 * c.q.word0 + q0 + lx0 + j];
            if (a > 0) {
                const unsigned long long k = cc_key(a, q0 + lx0 + j);
                key = k > key ? k : key;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned hi = __shfl_xor((unsigned)(key >> 32), o, 64), lo = __shfl_xor((unsigned)key, o, 64);
        const unsigned long long k = ((unsigned long long)hi << 32) | lo;
        key = k > key ? k : key;
    }
    unsigned long long *slot = &best[c.f];
    if ((tid & 63) == 0 && key && __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < key) atomicMax(slot, key);
}

struct PcRule {
    const int *labels, *area;
    const unsigned long long *best;
    int fill, min_area, keep_largest, max_hole_area;
};

// the opposite of store_row_word: the set bits of row-aligned word k of row y are CLEARED in the one or two flat words it covers
__device__ __forceinline__ void clear_row_word(uint32_t *op, int y, int W, int k, unsigned v)
{
    const long p = (long)y * W + 32 * k;
    const int o = (int)(p & 31);
    atomicAnd(&op[p >> 5], ~(v << o));
    const unsigned hi = o ? v >> (32 - o) : 0u;
    if (hi) atomicAnd(&op[(p >> 5) + 1], ~hi);
}

// fill = 0: the labels are those of the set pixels; a pixel whose component is not kept is cleared.  fill = 1: the labels are those of
// the zero pixels, with PC_BORDER in the area of a component that touches the border; a pixel of a hole of at most max_hole_area
// pixels is set.  Four adjacent threads make one row word; count[plane] += the pixels changed.
__global__ __launch_bounds__(CC_THREADS) void pc_apply_kernel(const long *__restrict__ plane, int P, long total_words,
                                                              const int *__restrict__ tiles, PcRule k, uint32_t *out, int *count)
{
    const PcTile c = pc_tile(tiles, plane, P, total_words);
    if (!c.ok) return;
    const int tid = threadIdx.x, W = c.q.W;
    const int ly = tid / (CC_TW / CC_PER), lx0 = (tid % (CC_TW / CC_PER)) * CC_PER;
    const long base = 32 * c.q.word0;
    unsigned m = 0u;
    if (ly < c.th) {
        const long g0 = base + (long)(c.y0 + ly) * W + c.x0;
        for (int j = 0; j < CC_PER && lx0 + j < c.tw; ++j) {
            const int root = k.labels[g0 + lx0 + j] - 1;
            if (root < 0) continue;
            const int a = k.area[base + root];
            const bool change = k.fill ? (a > 0 && a <= k.max_hole_area)
                                       : !(a >= k.min_area && (!k.keep_largest || k.best[c.f] == cc_key(a, root)));
            if (change) m |= 1u << j;
        }
    }
    int n = __popc(m);
    unsigned v = m << (8 * (tid & 3));
    v |= __shfl_xor(v, 1, 64);
    v |= __shfl_xor(v, 2, 64);
    if ((tid & 3) == 0 && v) {
        const int kw = (c.x0 + lx0) / 32;
        if (k.fill) store_row_word(out + c.q.word0, c.y0 + ly, W, kw, v, 0);
        else clear_row_word(out + c.q.word0, c.y0 + ly, W, kw, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((tid & 63) == 0 && n) atomicAdd(&count[c.f], n);
}

bool pc_sizes_ok(long total_words, int P) { return total_words >= 0 && P >= 0 && total_words < (1L << 50); }
long pc_slab_bytes(long total_words) { return (total_words * 128 + 15) / 16 * 16; }      // an i32 per pixel position of the buffer
template <typename T>
bool pc_aligned(const T *p) { return reinterpret_cast<uintptr_t>(p) % sizeof(T) == 0; }
uint8_t *pc_align16(void *p) { return reinterpret_cast<uint8_t *>((reinterpret_cast<uintptr_t>(p) + 15) / 16 * 16); }

// launches 1 to 3 for the pixels whose bit is `value`
void pc_label(const uint32_t *bits, const long *plane, int P, long total_words, unsigned value, int conn, const int *tiles, int n_tiles,
              int *parent, int *labels, int *area, int mark_border, hipStream_t stream)
{
    const dim3 grid((unsigned)n_tiles), block(CC_THREADS);
    hipLaunchKernelGGL(pc_tile_kernel, grid, block, 0, stream, bits, plane, P, total_words, tiles, value, conn == 8, parent, area);
    hipLaunchKernelGGL(pc_merge_kernel, grid, block, 0, stream, bits, plane, P, total_words, tiles, value, conn == 8, parent);
    hipLaunchKernelGGL(pc_flatten_kernel, grid, block, 0, stream, plane, P, total_words, tiles, parent, labels, area, mark_border);
}

}  // namespace

extern "C" {

int s2d_plane_components_tile(int *th, int *tw)
{
    if (!th || !tw) return S2D_ERR_ARG;
    *th = CC_TH;
    *tw = CC_TW;
    return S2D_OK;
}

long s2d_plane_components_workspace_bytes(long total_words, int P)
{
    if (!pc_sizes_ok(total_words, P)) return S2D_ERR_ARG;
    return 16 + 3 * pc_slab_bytes(total_words) + ((long)P * 8 + 15) / 16 * 16;     // 16: the workspace may start at any address
}

int s2d_plane_components_ragged(const uint32_t *bits, const long *plane, int P, long total_words, int value, int conn, const int *tiles,
                                int n_tiles, int *labels, int *area, void *workspace, hipStream_t stream)
{
    if (!pc_sizes_ok(total_words, P) || n_tiles < 0 || (value != 0 && value != 1) || (conn != 4 && conn != 8)) return S2D_ERR_ARG;
    if (!bits || !plane || !labels || !workspace || (n_tiles && !tiles)) return S2D_ERR_ARG;
    if (!pc_aligned(bits) || !pc_aligned(plane) || !pc_aligned(tiles) || !pc_aligned(labels) || !pc_aligned(area)) return S2D_ERR_ARG;
    // positions of no pixel hold 0
    if (total_words) {
        int rc = s2d_zero_async(labels, (size_t)total_words * 128, stream);
        if (rc == S2D_OK && area) rc = s2d_zero_async(area, (size_t)total_words * 128, stream);
        if (rc != S2D_OK) return rc;
    }
    if (P == 0 || n_tiles == 0 || total_words == 0) return S2D_OK;
    pc_label(bits, plane, P, total_words, (unsigned)value, conn, tiles, n_tiles, reinterpret_cast<int *>(pc_align16(workspace)), labels,
             area, 0, stream);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_plane_clean_ragged(const uint32_t *bits, const long *plane, int P, long total_words, int conn, int min_area, int keep_largest,
                           int max_hole_area, const int *tiles, int n_tiles, uint32_t *out, int *removed, int *filled, void *workspace,
                           hipStream_t stream)
{
    if (!pc_sizes_ok(total_words, P) || n_tiles < 0 || (conn != 4 && conn != 8) || min_area < 0 || max_hole_area < 0) return S2D_ERR_ARG;
    if (!bits || !plane || !out || !removed || !filled || !workspace || (n_tiles && !tiles)) return S2D_ERR_ARG;
    if (!pc_aligned(bits) || !pc_aligned(plane) || !pc_aligned(tiles) || !pc_aligned(out) || !pc_aligned(removed) || !pc_aligned(filled))
        return S2D_ERR_ARG;
    if (P == 0) return S2D_OK;
    int rc = s2d_zero_async(removed, (size_t)P * 4, stream);
    if (rc == S2D_OK) rc = s2d_zero_async(filled, (size_t)P * 4, stream);
    if (rc != S2D_OK) return rc;
    if (total_words == 0) return S2D_OK;
    hipLaunchKernelGGL(pc_copy_kernel, dim3((unsigned)P), dim3(256), 0, stream, bits, plane, total_words, out);
    uint8_t *ws = pc_align16(workspace);
    const long slab = pc_slab_bytes(total_words);
    int *parent = reinterpret_cast<int *>(ws), *labels = reinterpret_cast<int *>(ws + slab), *area = reinterpret_cast<int *>(ws + 2 * slab);
    unsigned long long *best = reinterpret_cast<unsigned long long *>(ws + 3 * slab);
    const dim3 grid((unsigned)n_tiles), block(CC_THREADS);
    // filter, then fill: the zero pixels are labelled in the FILTERED plane, so an island removed from inside a ring is filled with it
    if (n_tiles && (min_area > 0 || keep_largest)) {
        pc_label(out, plane, P, total_words, 1u, conn, tiles, n_tiles, parent, labels, area, 0, stream);
        if (keep_largest) {
            rc = s2d_zero_async(best, (size_t)P * 8, stream);
            if (rc != S2D_OK) return rc;
            hipLaunchKernelGGL(pc_best_kernel, grid, block, 0, stream, plane, P, total_words, tiles, area, best);
        }
        const PcRule rule = {labels, area, best, 0, min_area, keep_largest != 0, 0};
        hipLaunchKernelGGL(pc_apply_kernel, grid, block, 0, stream, plane, P, total_words, tiles, rule, out, removed);
    }
    if (n_tiles && max_hole_area > 0) {
        pc_label(out, plane, P, total_words, 0u, conn == 8 ? 4 : 8, tiles, n_tiles, parent, labels, area, 1, stream);
        const PcRule rule = {labels, area, best, 1, 0, 0, max_hole_area};
        hipLaunchKernelGGL(pc_apply_kernel, grid, block, 0, stream, plane, P, total_words, tiles, rule, out, filled);
    }
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

}  // extern "C"
