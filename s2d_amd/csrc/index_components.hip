// Connected components of u8 instance index maps (s2d_index_components_i32) and the integer cleanup rule on top of them
// (s2d_index_filter_components_u8): s2d_amd/index_components.py, DESIGN.md section 1.  The maps are what s2d_infer_paint_u8 and
// s2d_infer_index_u8 write: 0 = background, any other byte an instance id.  No plane per instance: all ids of a frame in one pass.
//
// Three launches, none of which waits for another workgroup:
//   1. cc_tile_kernel    a CC_TH x CC_TW tile per workgroup: union-find in LDS over tile-local offsets (< 2^16; held in 32-bit words,
//                        the width of an LDS atomic).  Every pixel gets parent = the raster index of its tile-local root (-1 on
//                        background); the root's area word gets the tile-local pixel count, every other area word 0.
//   2. cc_merge_kernel   a thread per pixel on the low side of a tile border: unions with its same-id neighbours across the border
//                        (for 8-connectivity the diagonal ones too, the contacts at tile corners among them).  parent[] is touched
//                        through agent-scope atomics only (relaxed loads, atomicMin): an L1 is never refreshed by another CU's
//                        stores.  A link only ever decreases, so a trip of any loop below either finishes or sees a strictly smaller
//                        parent (bounded by H*W), and the root of a component is its minimum raster index -- the canonical name.
//   3. cc_flatten_kernel a thread per pixel: walks to the root (plain loads: the launch boundary published the links),
//                        labels = 1 + root, and every tile-local root that is not the root moves its count there: one integer
//                        atomic per (tile, tile-local component).
// Integer sums and minima: the result does not depend on the order anything ran in, so a second call gives the same bits.
//
// The same three launches label the ZERO pixels (template parameter ZERO: one class, "the byte is 0") for the hole filling
// (s2d_index_fill_holes_u8; the rule: include/s2d_hip.h): fh_owner_kernel collects every zero component's owners and whether it
// touches the frame border, fh_fill_kernel writes the one-owner holes.  Again integer atomics only and no workgroup waits.
#include "components.h"

namespace {

constexpr int CC_WORDS = CC_TW / 4 + 1;                                  // aligned 4-byte words that cover a tile row at any address

// The pixels a call labels, as classes: pixels join where their classes are equal and not 0.  ZERO = false: the class is the id
// byte (the instances); ZERO = true: the zero pixels are the one class 1 and every instance pixel is 0 (the holes' labelling).
template <bool ZERO>
__device__ __forceinline__ uint8_t cc_class(uint8_t byte) { return ZERO ? (uint8_t)(byte == 0) : byte; }

// ---- launch 1 ----
template <bool ZERO>
__global__ __launch_bounds__(CC_THREADS) void cc_tile_kernel(const uint8_t *__restrict__ index, int H, int W, int tiles_x, int tiles_y,
                                                             int conn8, int *__restrict__ parent, int *__restrict__ area)
{
    __shared__ unsigned ids32[CC_TILE / 4];
    __shared__ unsigned par[CC_TILE];
    __shared__ unsigned cnt[CC_TILE];
    uint8_t *ids = reinterpret_cast<uint8_t *>(ids32);
    const int tid = threadIdx.x;
    const long blk = blockIdx.x;
    const int tx = (int)(blk % tiles_x), ty = (int)((blk / tiles_x) % tiles_y);
    const long n = blk / tiles_x / tiles_y;
    const int x0 = tx * CC_TW, y0 = ty * CC_TH;
    const int tw = min(CC_TW, W - x0), th = min(CC_TH, H - y0);
    const long HW = (long)H * W;
    const uint8_t *img = index + n * HW;

    // the tile's ids: aligned 4-byte words where a word lies inside the row segment, single bytes at its head and tail; nothing
    // outside [x0, x0 + tw) of a row is read.  Pixels of the tile past the image are background.
    for (int i = tid; i < CC_TILE / 4; i += CC_THREADS) ids32[i] = 0u;
    __syncthreads();
    for (int it = tid; it < th * CC_WORDS; it += CC_THREADS) {
        const int row = it / CC_WORDS, c = it % CC_WORDS;
        const uint8_t *a = img + (long)(y0 + row) * W + x0;
        const int off = 4 * c - (int)(reinterpret_cast<uintptr_t>(a) & 3);      // the word's first byte, relative to the segment
        if (off >= tw) continue;
        uint8_t *dst = ids + row * CC_TW;
        if (off >= 0 && off + 4 <= tw) {
            const unsigned v = *reinterpret_cast<const unsigned *>(a + off);
#pragma unroll
            for (int k = 0; k < 4; ++k) dst[off + k] = (uint8_t)(v >> (8 * k));
        } else {
            for (int k = 0; k < 4; ++k)
                if (off + k >= 0 && off + k < tw) dst[off + k] = a[off + k];
        }
    }
    __syncthreads();
    if (ZERO) {                                                          // classes in place; a tile position past the image is no pixel
        for (int i = tid; i < CC_TILE; i += CC_THREADS) ids[i] = (i / CC_TW < th && i % CC_TW < tw) ? cc_class<true>(ids[i]) : 0;
        __syncthreads();
    }

    // the union-find of the tile and the counts of its roots: components.h, shared with plane_components.hip
    const int ly = tid / (CC_TW / CC_PER), lx0 = (tid % (CC_TW / CC_PER)) * CC_PER;
    const unsigned i0 = ly * CC_TW + lx0;
    unsigned root[CC_PER];
    cc_tile_label(ids, par, cnt, conn8, root);
    if (ly >= th) return;
    const long row_g = (long)(y0 + ly) * W + x0;                         // < H*W < 2^31
    for (int j = 0; j < CC_PER; ++j) {
        const int lx = lx0 + j;
        if (lx >= tw) break;
        const long g = n * HW + row_g + lx;
        const unsigned r = root[j];
        parent[g] = r == CC_NONE ? -1 : (int)((long)(y0 + (int)(r / CC_TW)) * W + x0 + (int)(r % CC_TW));
        if (area) area[g] = r == i0 + j ? (int)cnt[r] : 0;
    }
}

// ---- launch 2 ----
// per image, nvb * H pixels on the right of a vertical tile border, then nhb * W pixels below a horizontal one.  A diagonal contact
// that crosses a vertical border belongs to the vertical part, the ones at tile corners included; the horizontal part takes the
// diagonals that stay inside a tile column.  Where the straight neighbour has the id, the diagonals beside it are joined through it.
template <bool ZERO>
__global__ __launch_bounds__(256) void cc_merge_kernel(const uint8_t *__restrict__ index, long total, int H, int W, int nvb, int nhb,
                                                       int conn8, int *parent)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const long HW = (long)H * W, per = (long)nvb * H + (long)nhb * W;
    const long n = t / per;
    long e = t % per;
    const uint8_t *img = index + n * HW;
    int *par = parent + n * HW;
    if (e < (long)nvb * H) {
        const int x = ((int)(e / H) + 1) * CC_TW, y = (int)(e % H);
        const int p = y * W + x;
        const uint8_t id = cc_class<ZERO>(img[p]);
        if (!id) return;
        if (cc_class<ZERO>(img[p - 1]) == id) {
            glb_union(par, p, p - 1);
        } else if (conn8) {
            // y % CC_TH == 0: the corner diagonal; (y + 1) % CC_TH == 0: the corner anti-diagonal
            if (y > 0 && cc_class<ZERO>(img[p - W - 1]) == id) glb_union(par, p, p - W - 1);
            if (y + 1 < H && cc_class<ZERO>(img[p + W - 1]) == id) glb_union(par, p, p + W - 1);
        }
    } else {
        e -= (long)nvb * H;
        const int y = ((int)(e / W) + 1) * CC_TH, x = (int)(e % W);
        const int p = y * W + x;
        const uint8_t id = cc_class<ZERO>(img[p]);
        if (!id) return;
        if (cc_class<ZERO>(img[p - W]) == id) {
            glb_union(par, p, p - W);
        } else if (conn8) {
            if (x % CC_TW != 0 && cc_class<ZERO>(img[p - W - 1]) == id) glb_union(par, p, p - W - 1);
            if ((x + 1) % CC_TW != 0 && x + 1 < W && cc_class<ZERO>(img[p - W + 1]) == id) glb_union(par, p, p - W + 1);
        }
    }
}

// ---- launch 3 ----
__global__ __launch_bounds__(256) void cc_flatten_kernel(const int *__restrict__ parent, long total, long HW, int *__restrict__ labels,
                                                         int *area)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const long base = t / HW * HW;
    const int q = (int)(t - base);
    int r = parent[t];
    if (r < 0) {
        labels[t] = 0;
        return;
    }
    for (int nx; (nx = parent[base + r]) != r;) r = nx;
    labels[t] = r + 1;
    // area[t] != 0: t is a tile-local root, and only this thread touches the word unless it is the root (then the others add to it)
    if (area && r != q) {
        const int c = area[t];
        if (c) {
            atomicAdd(&area[base + r], c);
            area[t] = 0;
        }
    }
}

// ---- the filter ----
// best[n][id] = max over the components of (image, id) of (area << 32) | ~first pixel: the largest, among equals the first.  One
// 64-bit atomicMax per root, in LDS: a workgroup covers 256 consecutive pixels of ONE image and keeps a table of its own, then
// sends each id it met to the global table once, unless the entry there already beats it (the table only grows, so a stale
// lower value read there only costs the atomic it could have saved).  A checkerboard -- every pixel a root of one id -- would
// otherwise queue H*W atomics on one address.
__global__ __launch_bounds__(256) void cc_best_kernel(const uint8_t *__restrict__ index, const int *__restrict__ area, long HW,
                                                      int blocks_per_image, unsigned long long *best)
{
    __shared__ unsigned long long local[256];
    const long n = blockIdx.x / blocks_per_image;
    const long p = (long)(blockIdx.x % blocks_per_image) * 256 + threadIdx.x;
    local[threadIdx.x] = 0ull;
    __syncthreads();
    if (p < HW) {
        const int a = area[n * HW + p];
        if (a > 0) atomicMax(&local[index[n * HW + p]], cc_key(a, (int)p));
    }
    __syncthreads();
    const unsigned long long key = local[threadIdx.x];
    unsigned long long *slot = &best[n * 256 + threadIdx.x];
    if (key && __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < key) atomicMax(slot, key);
}

struct CcRule {
    const int *labels, *area;
    const unsigned long long *best;
    int min_area, keep_largest;
    uint8_t *rgb;
    long HW;
};
// -> the output byte of pixel t = base + p of image n; a removed pixel blackens its rgb bytes and counts
__device__ __forceinline__ uint8_t cc_rule(const CcRule &k, long n, long base, long t, uint8_t id, int &removed)
{
    if (!id) return 0;
    const int root = k.labels[t] - 1;
    if (root < 0 || root >= k.HW) return id;                            // not a label of this map: nothing is looked up
    const int a = k.area[base + root];
    const bool keep = a >= k.min_area && (!k.keep_largest || k.best[n * 256 + id] == cc_key(a, root));
    if (keep) return id;
    ++removed;
    if (k.rgb) {
        uint8_t *c = k.rgb + 3 * t;
        c[0] = 0; c[1] = 0; c[2] = 0;
    }
    return 0;
}

// a thread per aligned 4-byte word of an image's index bytes: one 4-byte load where the word lies inside the image, single bytes
// at the image's head and tail; every thread reads its pixels before it writes them, so out may be index
__global__ __launch_bounds__(256) void cc_filter_kernel(const uint8_t *index, long HW, int blocks_per_image, CcRule k, uint8_t *out,
                                                        int *__restrict__ removed)
{
    __shared__ int part[4];
    const long n = blockIdx.x / blocks_per_image;
    const long g = (long)(blockIdx.x % blocks_per_image) * 256 + threadIdx.x;
    const long base = n * HW;
    const uint8_t *img = index + base;
    const long p0 = 4 * g - (long)(reinterpret_cast<uintptr_t>(img) & 3);
    int gone = 0;
    if (p0 >= 0 && p0 + 4 <= HW) {
        const unsigned v = *reinterpret_cast<const unsigned *>(img + p0);
        unsigned o = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) o |= (unsigned)cc_rule(k, n, base, base + p0 + j, (uint8_t)(v >> (8 * j)), gone) << (8 * j);
        uint8_t *dst = out + base + p0;
        if ((reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
            *reinterpret_cast<unsigned *>(dst) = o;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) dst[j] = (uint8_t)(o >> (8 * j));
        }
    } else if (p0 < HW) {
        uint8_t id[4];
        for (int j = 0; j < 4; ++j) id[j] = (p0 + j >= 0 && p0 + j < HW) ? img[p0 + j] : 0;
        for (int j = 0; j < 4; ++j)
            if (p0 + j >= 0 && p0 + j < HW) out[base + p0 + j] = cc_rule(k, n, base, base + p0 + j, id[j], gone);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) gone += __shfl_xor(gone, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = gone;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int s = part[0] + part[1] + part[2] + part[3];
        if (s) atomicAdd(&removed[n], s);
    }
}

// ---- the hole filling ----
// The zero pixels are labelled by the three launches above (ZERO = true) under the holes' connectivity.  fh_owner_kernel then gives
// every root owner_lo / owner_hi = the integer min / max of the ids of its pixels' non-zero neighbours, and every pixel on the frame
// border adds FH_BORDER (above any id) to owner_hi: a zero component is a hole with ONE owner iff owner_hi == owner_lo.  A
// workgroup covers 256 consecutive pixels of ONE image and aggregates in an LDS table keyed by the root (open addressing; 256 slots
// for at most 256 roots, so a probe always ends), then sends each root it met once, unless the global word already beats the value
// (the words only move one way, so a stale read only costs the atomic it could have saved).  A frame-sized hole has thousands of
// boundary pixels for ONE root: they would otherwise queue on one address.
constexpr int FH_BORDER = 256;
constexpr int FH_NONE = 0x7fffffff;                                     // owner_lo before any owner

__global__ __launch_bounds__(256) void fh_init_kernel(long total, int *__restrict__ owner_lo, int *__restrict__ owner_hi)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    owner_lo[t] = FH_NONE;
    owner_hi[t] = 0;
}

__global__ __launch_bounds__(256) void fh_owner_kernel(const uint8_t *__restrict__ index, const int *__restrict__ labels, int H, int W,
                                                       int blocks_per_image, int conn8, int *owner_lo, int *owner_hi)
{
    __shared__ int key[256], lo[256], hi[256];
    const long HW = (long)H * W;
    const long n = blockIdx.x / blocks_per_image;
    const long p = (long)(blockIdx.x % blocks_per_image) * 256 + threadIdx.x;
    key[threadIdx.x] = -1;
    lo[threadIdx.x] = FH_NONE;
    hi[threadIdx.x] = 0;
    __syncthreads();
    const uint8_t *img = index + n * HW;
    if (p < HW && img[p] == 0) {
        const int y = (int)(p / W), x = (int)(p % W);
        int mlo = FH_NONE, mhi = (y == 0 || y == H - 1 || x == 0 || x == W - 1) ? FH_BORDER : 0;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                if ((!dy && !dx) || (!conn8 && dy && dx)) continue;
                const int yy = y + dy, xx = x + dx;
                if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                const int id = img[(long)yy * W + xx];
                if (id) {
                    mlo = min(mlo, id);
                    mhi = max(mhi, id);
                }
            }
        if (mhi) {                                                       // a pixel inside its hole has nothing to say
            const int root = labels[n * HW + p] - 1;
            unsigned s = (unsigned)root & 255u;
            for (;;) {
                const int old = atomicCAS(&key[s], -1, root);
                if (old == -1 || old == root) break;
                s = (s + 1) & 255u;
            }
            atomicMin(&lo[s], mlo);
            atomicMax(&hi[s], mhi);
        }
    }
    __syncthreads();
    const int root = key[threadIdx.x];
    if (root >= 0) {
        int *glo = owner_lo + n * HW + root, *ghi = owner_hi + n * HW + root;
        const int l = lo[threadIdx.x], h = hi[threadIdx.x];
        if (__hip_atomic_load(ghi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < h) atomicMax(ghi, h);
        if (__hip_atomic_load(glo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > l) atomicMin(glo, l);
    }
}

struct FhRule {
    const int *labels, *area, *owner_lo, *owner_hi;
    int max_area, n_colors;
    uint8_t *rgb;
    const uint8_t *colors;
};
// -> the output byte of pixel t of the image that starts at base; a filled pixel takes its owner's colour and counts.  owner_hi ==
// owner_lo holds for ids 1..255 alone: 0 and FH_BORDER are no value of owner_lo, FH_NONE none of owner_hi.
__device__ __forceinline__ uint8_t fh_rule(const FhRule &k, long base, long t, uint8_t id, int &filled)
{
    if (id) return id;
    const long r = base + k.labels[t] - 1;
    const int owner = k.owner_hi[r];
    if (owner != k.owner_lo[r] || k.area[r] > k.max_area) return 0;
    if (k.rgb) {
        if (owner > k.n_colors) return 0;                                // no colour for it: left alone in map and picture
        uint8_t *c = k.rgb + 3 * t;
        const uint8_t *s = k.colors + 3 * (owner - 1);
        c[0] = s[0]; c[1] = s[1]; c[2] = s[2];
    }
    ++filled;
    return (uint8_t)owner;
}

// a thread per aligned 4-byte word of an image's index bytes, as cc_filter_kernel: every thread reads its pixels before it writes
// them, so out may be index
__global__ __launch_bounds__(256) void fh_fill_kernel(const uint8_t *index, long HW, int blocks_per_image, FhRule k, uint8_t *out,
                                                      int *__restrict__ filled)
{
    __shared__ int part[4];
    const long n = blockIdx.x / blocks_per_image;
    const long g = (long)(blockIdx.x % blocks_per_image) * 256 + threadIdx.x;
    const long base = n * HW;
    const uint8_t *img = index + base;
    const long p0 = 4 * g - (long)(reinterpret_cast<uintptr_t>(img) & 3);
    int set = 0;
    if (p0 >= 0 && p0 + 4 <= HW) {
        const unsigned v = *reinterpret_cast<const unsigned *>(img + p0);
        unsigned o = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) o |= (unsigned)fh_rule(k, base, base + p0 + j, (uint8_t)(v >> (8 * j)), set) << (8 * j);
        uint8_t *dst = out + base + p0;
        if ((reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
            *reinterpret_cast<unsigned *>(dst) = o;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) dst[j] = (uint8_t)(o >> (8 * j));
        }
    } else if (p0 < HW) {
        uint8_t id[4];
        for (int j = 0; j < 4; ++j) id[j] = (p0 + j >= 0 && p0 + j < HW) ? img[p0 + j] : 0;
        for (int j = 0; j < 4; ++j)
            if (p0 + j >= 0 && p0 + j < HW) out[base + p0 + j] = fh_rule(k, base, base + p0 + j, id[j], set);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) set += __shfl_xor(set, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = set;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int s = part[0] + part[1] + part[2] + part[3];
        if (s) atomicAdd(&filled[n], s);
    }
}

bool cc_dims_ok(int N, int H, int W) { return N >= 1 && H >= 1 && W >= 1 && (long)H * W < 2147483647L; }
long cc_parent_bytes(int N, int H, int W) { return ((long)N * H * W * 4 + 15) / 16 * 16; }
template <typename T>
bool cc_aligned(const T *p) { return reinterpret_cast<uintptr_t>(p) % sizeof(T) == 0; }
uint8_t *cc_align16(void *p) { return reinterpret_cast<uint8_t *>((reinterpret_cast<uintptr_t>(p) + 15) / 16 * 16); }

// the three launches: the components of the classes of cc_class<ZERO>.  parent: N*H*W words of scratch
template <bool ZERO>
int cc_label(const uint8_t *index, int N, int H, int W, int conn8, int *labels, int *area, int *parent, hipStream_t stream)
{
    const long HW = (long)H * W, total = (long)N * HW;
    const int tiles_x = cdiv(W, CC_TW), tiles_y = cdiv(H, CC_TH), nvb = (W - 1) / CC_TW, nhb = (H - 1) / CC_TH;
    const long tiles = (long)N * tiles_x * tiles_y, border = (long)N * ((long)nvb * H + (long)nhb * W);
    if (tiles > 2147483647L || (total + 255) / 256 > 2147483647L) return S2D_ERR_ARG;
    hipLaunchKernelGGL(cc_tile_kernel<ZERO>, dim3((unsigned)tiles), dim3(CC_THREADS), 0, stream, index, H, W, tiles_x, tiles_y, conn8,
                       parent, area);
    if (border > 0)
        hipLaunchKernelGGL(cc_merge_kernel<ZERO>, dim3((unsigned)((border + 255) / 256)), dim3(256), 0, stream, index, border, H, W, nvb,
                           nhb, conn8, parent);
    hipLaunchKernelGGL(cc_flatten_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, parent, total, HW, labels, area);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

}  // namespace

extern "C" {

int s2d_index_components_tile(int *th, int *tw)
{
    if (!th || !tw) return S2D_ERR_ARG;
    *th = CC_TH;
    *tw = CC_TW;
    return S2D_OK;
}

long s2d_index_components_workspace_bytes(int N, int H, int W)
{
    if (!cc_dims_ok(N, H, W)) return S2D_ERR_ARG;
    return 16 + cc_parent_bytes(N, H, W) + (long)N * 256 * 8;            // 16: the workspace may start at any address
}

int s2d_index_components_i32(const uint8_t *index, int N, int H, int W, int conn, int *labels, int *area, void *workspace,
                             hipStream_t stream)
{
    if (!cc_dims_ok(N, H, W) || (conn != 4 && conn != 8) || !index || !labels || !workspace) return S2D_ERR_ARG;
    if (!cc_aligned(labels) || !cc_aligned(area)) return S2D_ERR_ARG;
    return cc_label<false>(index, N, H, W, conn == 8, labels, area, reinterpret_cast<int *>(cc_align16(workspace)), stream);
}

int s2d_index_filter_components_u8(const uint8_t *index, const int *labels, const int *area, int N, int H, int W, int min_area,
                                   int keep_largest, uint8_t *out, uint8_t *rgb, int *removed, void *workspace, hipStream_t stream)
{
    if (!cc_dims_ok(N, H, W) || min_area < 0 || !index || !labels || !area || !out || !removed || !workspace) return S2D_ERR_ARG;
    if (!cc_aligned(labels) || !cc_aligned(area) || !cc_aligned(removed)) return S2D_ERR_ARG;
    const long HW = (long)H * W;
    const int blocks_per_image = cdiv((HW + 3 + 3) / 4, 256);            // words that cover HW bytes at any address
    const int best_blocks = cdiv(HW, 256);                               // 256 pixels of one image per workgroup
    if ((long)N * blocks_per_image > 2147483647L || (long)N * best_blocks > 2147483647L) return S2D_ERR_ARG;
    unsigned long long *best = reinterpret_cast<unsigned long long *>(cc_align16(workspace) + cc_parent_bytes(N, H, W));
    int rc = s2d_zero_async(removed, (size_t)N * 4, stream);
    if (rc != S2D_OK) return rc;
    if (keep_largest) {
        rc = s2d_zero_async(best, (size_t)N * 256 * 8, stream);
        if (rc != S2D_OK) return rc;
        hipLaunchKernelGGL(cc_best_kernel, dim3((unsigned)((long)N * best_blocks)), dim3(256), 0, stream, index, area, HW, best_blocks,
                           best);
    }
    const CcRule rule = {labels, area, best, min_area, keep_largest != 0, rgb, HW};
    hipLaunchKernelGGL(cc_filter_kernel, dim3((unsigned)((long)N * blocks_per_image)), dim3(256), 0, stream, index, HW, blocks_per_image,
                       rule, out, removed);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

long s2d_index_fill_holes_workspace_bytes(int N, int H, int W)
{
    if (!cc_dims_ok(N, H, W)) return S2D_ERR_ARG;
    return 16 + 4 * cc_parent_bytes(N, H, W);                            // parent (then owner_hi), labels, area, owner_lo
}

int s2d_index_fill_holes_u8(const uint8_t *index, int N, int H, int W, int conn, int max_hole_area, uint8_t *out, uint8_t *rgb,
                            const uint8_t *colors, int n_colors, int *filled, void *workspace, hipStream_t stream)
{
    if (!cc_dims_ok(N, H, W) || (conn != 4 && conn != 8) || max_hole_area < 1 || !index || !out || !filled || !workspace)
        return S2D_ERR_ARG;
    if (rgb && (!colors || n_colors < 1 || n_colors > 255)) return S2D_ERR_ARG;
    if (!cc_aligned(filled)) return S2D_ERR_ARG;
    const long HW = (long)H * W, total = (long)N * HW, words = cc_parent_bytes(N, H, W) / 4;
    const int blocks_per_image = cdiv((HW + 3 + 3) / 4, 256);            // words that cover HW bytes at any address
    const int owner_blocks = cdiv(HW, 256);                              // 256 pixels of one image per workgroup
    if ((long)N * blocks_per_image > 2147483647L || (long)N * owner_blocks > 2147483647L) return S2D_ERR_ARG;
    if ((long)N * cdiv(W, CC_TW) * cdiv(H, CC_TH) > 2147483647L) return S2D_ERR_ARG;      // cc_label's grids, before the first launch
    int *parent = reinterpret_cast<int *>(cc_align16(workspace));
    int *labels = parent + words, *area = labels + words, *owner_lo = area + words;
    int rc = s2d_zero_async(filled, (size_t)N * 4, stream);
    if (rc != S2D_OK) return rc;
    const int hole_conn8 = conn == 4;                                    // the complementary connectivity
    rc = cc_label<true>(index, N, H, W, hole_conn8, labels, area, parent, stream);
    if (rc != S2D_OK) return rc;
    int *owner_hi = parent;                                              // the links are spent once the labels are written
    hipLaunchKernelGGL(fh_init_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, total, owner_lo, owner_hi);
    hipLaunchKernelGGL(fh_owner_kernel, dim3((unsigned)((long)N * owner_blocks)), dim3(256), 0, stream, index, labels, H, W, owner_blocks,
                       hole_conn8, owner_lo, owner_hi);
    const FhRule rule = {labels, area, owner_lo, owner_hi, max_hole_area, rgb ? n_colors : 0, rgb, colors};
    hipLaunchKernelGGL(fh_fill_kernel, dim3((unsigned)((long)N * blocks_per_image)), dim3(256), 0, stream, index, HW, blocks_per_image,
                       rule, out, filled);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

}  // extern "C"
